"""CPU: the ticket -> (chunk, hypothesis) arithmetic of houv_solve_stage and an item's steps_done / length (houv_math.h, compiled
for the host): chunk-major tickets, every (hypothesis, iteration) of the stage covered exactly once and in order, the last chunk
what is left -- the same cuts solver.run_stage's loop of separate launches makes."""
from tests import schedmath

SHAPES = [(1, 1, 1), (1, 7, 3), (6, 7, 3), (7, 5, 2), (8, 6, 3), (8, 6, 8), (5, 200, 50), (3, 199, 50), (2, 4, 2 ** 31 - 1),
          (3, 50, 50), (4, 51, 50)]


def test_tickets_cover_every_iteration_once_in_chunk_major_order():
    for (ninst, n_iters, chunk), (items, items64, chunks, rows) in zip(SHAPES, schedmath.items(SHAPES)):
        cuts, done = [], 0
        while done < n_iters:                               # run_stage's loop
            it = min(chunk, n_iters - done)
            cuts.append((done, it))
            done += it
        assert chunks == len(cuts) and items == items64 == ninst * chunks and len(rows) == items
        for t, (ticket, c, h, steps, iters) in enumerate(rows):
            assert ticket == t and c == t // ninst and h == t % ninst
            assert (steps, iters) == cuts[c] and iters >= 1
        # chunk-major: the earlier chunk of a hypothesis was drawn exactly ninst tickets before
        for t in range(ninst, items):
            assert rows[t - ninst][1:3] == (rows[t][1] - 1, rows[t][2])
