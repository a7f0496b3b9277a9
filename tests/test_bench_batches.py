"""bench.py makes the synthetic batches of a large run in worker processes: they have to be synthetic.make_pairs' batches
bit for bit, whatever the split into jobs."""
import torch

import bench
from houv_amd import synthetic


def test_host_batches_equal_make_pairs():
    first_ids = [0, 40, 13]                          # 20 pairs per batch: one full job of 16 pairs and a ragged one of 4
    got = bench.host_batches(20, 192, first_ids, min_pairs=0)
    assert len(got) == len(first_ids)
    for f, batch in zip(first_ids, got):
        want = synthetic.make_pairs(20, 192, seed=2021, first_id=f)
        for w, g in zip(want, batch):
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w)
