"""Host-side scheduler of ``IterativeSolver.solve_many``: continuous batching for the solver.

A job of N maps runs in ``slots`` rows of the batch arrays.  After every chunk of iterations the device leaves one verdict record per
active slot (``hn_stream_verdict``); this module turns those records into the operation list of ``hn_stream_swap`` -- which slots are
retired into the job's output rows, which take the next unsolved map, and, once no map is left, which tail slots are moved into the holes
so that the solver always iterates a dense prefix ``[0, active)``.

Pure Python on purpose (no torch, no shared library): the scheduling rules are tested on the CPU against a scripted table of
"iterations each map needs" (tests/test_stream_host.py).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

CONVERGED, MAX_ITERATIONS, DIVERGED = 0, 1, 2

# (slot, retire_map, move_from, refill_map), -1 = none: struct hn_stream_op of include/helmnet_hip.h
Op = Tuple[int, int, int, int]


class StreamScheduler:
    """State of one ``solve_many`` job.

        sched = StreamScheduler(n_maps, slots, max_iterations, check_every)
        ops = sched.initial_ops()                      # refill-only: the first min(slots, n_maps) maps
        while sched.active:
            chunk = sched.next_chunk()                 # iterations to run on slots [0, sched.active)
            ... run them, obtain one (first_below, bad, last_rmse) record per active slot ...
            ops = sched.advance(chunk, records)        # retire / refill / move; updates sched.active

    Rules.  A map is retired after the chunk in which its record is ``bad`` (status 2), else in which its RMSE was below the tolerance at
    some iteration (``first_below >= 0``, status 0), else once it has run ``max_iterations`` (status 1).  Chunks are ``check_every`` long,
    shortened to what the active map closest to ``max_iterations`` has left -- so every iteration count is a multiple of ``check_every``
    capped at ``max_iterations`` whenever ``max_iterations`` is itself a multiple (otherwise the maps in flight during a shortened chunk
    carry its remainder).  ``sample_iterations`` counts the work enqueued: the sum over chunks of active slots x chunk length.
    """

    def __init__(self, n_maps: int, slots: int, max_iterations: int, check_every: int):
        if n_maps < 0:
            raise ValueError("n_maps must not be negative")
        if slots < 1 or max_iterations < 1 or check_every < 1:
            raise ValueError("slots, max_iterations and check_every must be positive")
        self.n_maps, self.slots = int(n_maps), int(slots)
        self.max_iterations, self.check_every = int(max_iterations), int(check_every)
        self.slot_map: List[int] = []        # map solved in slot s, for s in [0, active)
        self.slot_done: List[int] = []       # iterations that map has run
        self.next_map = 0
        self.iterations = [0] * self.n_maps
        self.status = [-1] * self.n_maps
        self.residual_norm = [float("nan")] * self.n_maps
        self.sample_iterations = 0
        self.chunks = 0

    @property
    def active(self) -> int:
        return len(self.slot_map)

    def initial_ops(self) -> List[Op]:
        if self.slot_map or self.next_map:
            raise RuntimeError("initial_ops() is the first call of a job")
        ops = []
        for s in range(min(self.slots, self.n_maps)):
            ops.append((s, -1, -1, self.next_map))
            self.slot_map.append(self.next_map)
            self.slot_done.append(0)
            self.next_map += 1
        return ops

    def next_chunk(self) -> int:
        if not self.slot_map:
            return 0
        return min(self.check_every, self.max_iterations - max(self.slot_done))

    def advance(self, chunk: int, records: Sequence[Sequence]) -> List[Op]:
        """``records[s]`` = (first_below, bad, last_rmse) of slot s for the ``chunk`` iterations just run on slots [0, active)."""
        active = self.active
        if len(records) < active:
            raise ValueError(f"{len(records)} verdict records for {active} active slots")
        if chunk < 1 or chunk > self.next_chunk():
            raise ValueError(f"chunk of {chunk} iterations (at most {self.next_chunk()})")
        self.sample_iterations += active * chunk
        self.chunks += 1
        ops: List[Op] = []
        holes: List[Tuple[int, int]] = []    # (slot, retired map) once no map is left to refill with
        for s in range(active):
            first_below, bad, last_rmse = records[s][0], records[s][1], records[s][2]
            self.slot_done[s] += chunk
            if bad:
                status = DIVERGED
            elif first_below >= 0:
                status = CONVERGED
            elif self.slot_done[s] >= self.max_iterations:
                status = MAX_ITERATIONS
            else:
                continue
            m = self.slot_map[s]
            self.iterations[m], self.status[m], self.residual_norm[m] = self.slot_done[s], status, float(last_rmse)
            if self.next_map < self.n_maps:
                ops.append((s, m, -1, self.next_map))
                self.slot_map[s], self.slot_done[s] = self.next_map, 0
                self.next_map += 1
            else:
                holes.append((s, m))
        if holes:
            # tail compaction: the last surviving slots move into the holes below the new end of the prefix; a mover is only read by
            # this launch (it is neither a hole nor refilled), a hole at or beyond the new end is only retired
            new_active = active - len(holes)
            hole_slots = {s for s, _ in holes}
            movers = [s for s in range(active - 1, new_active - 1, -1) if s not in hole_slots]
            for s, m in holes:
                if s < new_active:
                    src = movers.pop(0)
                    ops.append((s, m, src, -1))
                    self.slot_map[s], self.slot_done[s] = self.slot_map[src], self.slot_done[src]
                else:
                    ops.append((s, m, -1, -1))
            assert not movers
            del self.slot_map[new_active:], self.slot_done[new_active:]
        return ops
