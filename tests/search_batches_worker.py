"""Worker of tests/test_gpu_search.py::test_flat_many_small_batches: the library reads FALCON_SIMS_MB once per process, so the
batch cuts of a search run in a fresh process that has it set to 16 (a hand-off buffer of 4,194,304 floats).  Low_dim 64.
Never imported by pytest."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_SIMS_MB") == "16"
    import torch
    from falcon_amd.device import Context
    from oracle import falcon_oracle as fo
    from tests import search_cases as sc
    from tests import test_gpu_ivf16 as t16
    from tests.test_gpu_search import unit_vectors
    from tests.util import assert_topk_exact
    ctx = Context(0)

    # (a) flat: nine buckets of 1,000 rows (1,048,576 floats each: batches of 4, 4 and the rest), three of 20 rows, two of 300
    sizes = sc.GPU_FLAT_SIZES
    off = np.concatenate([[0], np.cumsum(sizes)])
    X = unit_vectors(off[-1], 64, 5)
    idxr = ctx.ivf_build(torch.from_numpy(X).to(ctx.tdev), off, np.ones(len(sizes), np.int32))
    sim, idx = idxr.search(16, 32)
    sim, idx = sim.cpu().numpy(), idx.cpu().numpy()
    assert ctx.counter(2) == sc.GPU_FLAT_BATCHES, ctx.counter(2)
    for a, b in zip(off[:-1], off[1:]):
        rs, ri = fo.exhaustive_topk(X[a:b], 32, base=a)
        assert_topk_exact(sim[a:b], idx[a:b], rs, ri, what=f"flat bucket {a}:{b}")
    print("ok flat", flush=True)

    # (b) indexed, staged: two buckets of 3,000 rows, every list probed -- 9 M candidates a bucket, more than the buffer holds:
    # the fine scan runs bucket by bucket, and brute force is the oracle
    sizes, nl = [3000, 3000], np.array([16, 16], np.int32)
    off, X, mz, _ = t16._buckets(sizes, 64, 57)
    idxr = ctx.ivf_build(torch.from_numpy(X).to(ctx.tdev), off, nl)
    sim, idx = idxr.search(16, 64)
    sim, idx = sim.cpu().numpy(), idx.cpu().numpy()
    assert ctx.counter(2) == 0 + 2, ctx.counter(2)                 # no flat batch + two fine batches
    for a, b in zip(off[:-1], off[1:]):
        rs, ri = fo.exhaustive_topk(X[a:b], 64, base=a)
        assert_topk_exact(sim[a:b], idx[a:b], rs, ri, what=f"indexed bucket {a}:{b}")
    print("ok staged", flush=True)

    # (c) indexed, float16 prefilter attached: a batch of 16-bit keys holds twice the candidates, 8,388,608 -- still fewer than a
    # bucket's 9 M.  Neighbour lists bit for bit those of the staged path
    _, n_fb = t16._staged_and_prefiltered(ctx, X, off, nl, mz, None, 16, 64, 16, 20.0, "ppm", None)
    assert ctx.counter(2) == 0 + 2, ctx.counter(2)
    assert n_fb < 0.05 * off[-1], n_fb
    print("batches ok", flush=True)


if __name__ == "__main__":
    main()
