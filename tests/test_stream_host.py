"""CPU-only checks of the solve_many layer: the two C entry points are declared, exported and bound, and the scheduler that turns verdict
records into hn_stream_swap operation lists obeys its rules on a scripted table of "iterations each map needs" (no GPU, no kernels)."""
import os
import re

import pytest

from helmnet_amd.stream_schedule import CONVERGED, DIVERGED, MAX_ITERATIONS, StreamScheduler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_symbols_declared_exported_and_bound():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    declared = set(re.findall(r"\b(hn_[a-z_0-9]+)\s*\(", hdr))
    for name in ("hn_stream_verdict", "hn_stream_swap"):
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert len(_lib.SYMBOLS["hn_stream_verdict"][1]) == 8 and len(_lib.SYMBOLS["hn_stream_swap"][1]) == 17
    for struct, fields in (("hn_stream_verdict_rec", "int32_t first_below; int32_t bad; float last_rmse;"),
                           ("hn_stream_op", "int32_t slot, retire_map, move_from, refill_map;")):
        assert re.search(r"typedef struct %s \{ %s \} %s;" % (struct, re.escape(fields), struct), hdr), struct
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # new entry points within ABI 7
    # without a context both calls fail cleanly
    assert lib.hn_stream_verdict(None, None, 1, 1, 0.0, 0.0, None, None) == -1
    assert lib.hn_stream_swap(None, None, None, None, None, None, 1, 1, 0, None, None, None, 0, 1.0, None, None, None) == -1


def test_verdict_record_layout_matches_the_header():
    from helmnet_amd.engine import Engine
    dt = Engine.VERDICT_DTYPE
    assert dt.itemsize == 12 and dt.names == ("first_below", "bad", "last_rmse")
    assert [dt.fields[k][1] for k in dt.names] == [0, 4, 8]


def _drive(needs, slots, max_iterations, check_every, bad=()):
    """Run the scheduler against a model of the device: map m's RMSE is below tol from iteration needs[m] on (None: never); maps in
    ``bad`` produce a non-finite RMSE in their first chunk.  Mirrors the slot arrays hn_stream_swap acts on and checks every launch."""
    n_maps = len(needs)
    sched = StreamScheduler(n_maps, slots, max_iterations, check_every)
    slot_map = {}                      # the model's own view of which map sits in which slot, maintained from the ops alone
    slot_done = {}
    retired = {}

    def apply(ops):
        slots_named = [o[0] for o in ops]
        assert len(set(slots_named)) == len(slots_named), "a slot is named twice"
        written = {o[0] for o in ops if o[2] >= 0 or o[3] >= 0}
        for s, ret, frm, fill in ops:
            assert 0 <= s < slots
            assert not (frm >= 0 and fill >= 0)
            if frm >= 0:
                assert frm != s and frm not in written, "a launch reads a slot it writes"
                assert frm in slot_map
        before = dict(slot_map), dict(slot_done)
        for s, ret, frm, fill in ops:
            if ret >= 0:
                assert before[0][s] == ret, "retired map is not the one in the slot"
                assert ret not in retired, "map retired twice"
                retired[ret] = before[1][s]
                slot_map.pop(s), slot_done.pop(s)
            if frm >= 0:
                slot_map[s], slot_done[s] = before[0][frm], before[1][frm]
            if fill >= 0:
                assert 0 <= fill < n_maps
                slot_map[s], slot_done[s] = fill, 0
        # a mover's old slot is beyond the new prefix: drop it from the model
        for s in [s for s in slot_map if s >= sched.active]:
            assert any(o[2] == s for o in ops), "a live slot fell off the prefix without being moved"
            slot_map.pop(s), slot_done.pop(s)
        assert sorted(slot_map) == list(range(sched.active)), "the active prefix is not dense"
        assert [slot_map[s] for s in range(sched.active)] == sched.slot_map
        assert [slot_done[s] for s in range(sched.active)] == sched.slot_done

    first = sched.initial_ops()
    assert all(o[1] == -1 and o[2] == -1 for o in first) and [o[3] for o in first] == list(range(min(slots, n_maps)))
    apply(first)
    work, guard = 0, 0
    while sched.active:
        guard += 1
        assert guard < 100000
        a, chunk = sched.active, sched.next_chunk()
        assert 1 <= chunk <= check_every
        records = []
        for s in range(a):
            m, d0 = slot_map[s], slot_done[s]
            assert d0 + chunk <= max_iterations
            need = needs[m]
            fb = -1 if need is None or need > d0 + chunk else max(need - d0 - 1, 0)
            records.append((fb, 1 if m in bad else 0, 1.0))
            slot_done[s] = d0 + chunk
        work += a * chunk
        apply(sched.advance(chunk, records))
    assert sorted(retired) == list(range(n_maps)), "every map is retired exactly once"
    assert sched.sample_iterations == work
    assert all(retired[m] == sched.iterations[m] for m in range(n_maps))
    return sched


def _expected_iterations(need, max_iterations, check_every):
    if need is None or need > max_iterations:
        return max_iterations, MAX_ITERATIONS
    return min(-(-need // check_every) * check_every, max_iterations), CONVERGED


@pytest.mark.parametrize("slots", [1, 3, 8, 32])
def test_scheduler_against_a_scripted_table(slots):
    needs = [30, 180, 7, 25, 26, 99, 100, 101, None, 55, 240, 12, 75, 130, 61, 200, 18, 49, 51, 88, 300]
    sched = _drive(needs, slots, max_iterations=250, check_every=25)
    want = [_expected_iterations(nd, 250, 25) for nd in needs]
    assert sched.iterations == [w[0] for w in want]
    assert sched.status == [w[1] for w in want]
    # the analytic sum: with max_iterations a multiple of check_every every chunk is full, so the work enqueued is the iterations delivered
    assert sched.sample_iterations == sum(w[0] for w in want)
    # ... strictly less than the batch-wise loop (every batch runs until its worst map is done) whenever a batch holds unequal maps
    batchwise = sum(len(needs[i:i + slots]) * max(w[0] for w in want[i:i + slots]) for i in range(0, len(needs), slots))
    assert sched.sample_iterations < batchwise or slots == 1


def test_scheduler_fewer_maps_than_slots_and_empty_job():
    sched = _drive([40, 10, 90], slots=8, max_iterations=100, check_every=25)
    assert sched.iterations == [50, 25, 100] and sched.status == [CONVERGED] * 3
    assert sched.sample_iterations == 3 * 25 + 2 * 25 + 1 * 50
    empty = StreamScheduler(0, 8, 100, 25)
    assert empty.initial_ops() == [] and empty.active == 0 and empty.next_chunk() == 0
    assert empty.iterations == [] and empty.status == [] and empty.sample_iterations == 0


def test_scheduler_max_iterations_not_a_multiple_of_check_every():
    # one slot: chunks of 25, 25, 10 for a map that never converges; 60 is never exceeded
    sched = _drive([None, 30], slots=1, max_iterations=60, check_every=25)
    assert sched.iterations == [60, 50] and sched.status == [MAX_ITERATIONS, CONVERGED]
    assert sched.sample_iterations == 60 + 50
    # several slots of different ages: a shortened chunk applies to every active slot, nobody runs past max_iterations, the sum stays exact
    needs = [None, 20, None, 55, 58, None, 3]
    sched = _drive(needs, slots=3, max_iterations=60, check_every=25)
    assert all(it <= 60 for it in sched.iterations)
    for m, nd in enumerate(needs):
        if nd is None:
            assert (sched.iterations[m], sched.status[m]) == (60, MAX_ITERATIONS)
        else:
            assert sched.status[m] == CONVERGED and nd <= sched.iterations[m] < nd + 25
    assert sched.sample_iterations == sum(sched.iterations)


def test_scheduler_bad_records_take_precedence_and_retire_after_one_chunk():
    needs = [10, 40, None, 30, 5]
    sched = _drive(needs, slots=2, max_iterations=50, check_every=25, bad={0, 2})
    assert sched.status == [DIVERGED, CONVERGED, DIVERGED, CONVERGED, CONVERGED]
    assert sched.iterations == [25, 50, 25, 50, 25]


def test_scheduler_rejects_bad_arguments():
    for args in ((-1, 8, 100, 25), (4, 0, 100, 25), (4, 8, 0, 25), (4, 8, 100, 0)):
        with pytest.raises(ValueError):
            StreamScheduler(*args)
    sched = StreamScheduler(2, 2, 100, 25)
    sched.initial_ops()
    with pytest.raises(ValueError):
        sched.advance(25, [(-1, 0, 1.0)])        # one record for two active slots
    with pytest.raises(ValueError):
        sched.advance(26, [(-1, 0, 1.0)] * 2)    # longer than the chunk the scheduler asked for
