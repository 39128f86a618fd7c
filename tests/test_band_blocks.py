"""CPU checks of graph.band_blocks, the host plan of the banded round (runs without a GPU)."""
import numpy as np
import pytest


def ring(n):
    from distributed_learning_amd.graph import Csr
    cols = np.concatenate([[a, (a + 1) % n, (a - 1) % n] for a in range(n)])
    return Csr(np.arange(0, 3 * n + 1, 3), cols, np.full(3 * n, 1 / 3))


def torus(r, c):
    from distributed_learning_amd import graph
    return graph.uniform_weights(graph.torus_edges(r, c), 0.2, list(range(r * c)))


def banded(n, seed=0):
    """Rows of 2-9 entries: self and random neighbours within +-7 (wrapping), scrambled order,
    row-stochastic per-entry weights."""
    from distributed_learning_amd.graph import Csr
    rng = np.random.default_rng(seed)
    rp, cl, w = [0], [], []
    for a in range(n):
        off = rng.permutation(np.r_[-7:0, 1:8])[:rng.integers(1, 9)]
        nb = rng.permutation(np.r_[a, (a + off) % n])
        wt = rng.random(len(nb)) + 0.1
        cl.extend(nb.tolist())
        w.extend((wt / wt.sum()).tolist())
        rp.append(len(cl))
    return Csr(rp, cl, w)


@pytest.mark.parametrize("make,cap,segments", [(lambda: ring(300), 48, 2),
                                               (lambda: torus(12, 25), 60, 3),
                                               (lambda: banded(300), 48, 2)])
def test_slots_segments_and_promises(make, cap, segments):
    from distributed_learning_amd.graph import band_blocks
    csr = make()
    p = band_blocks(csr, cap, tile_cols=16, max_amplification=8.0)
    assert p.block_row[0] == 0 and p.block_row[-1] == csr.n_rows and np.all(np.diff(p.block_row) > 0)
    assert p.blocks > 3 and len(set(np.diff(p.block_row))) > 1            # a ragged last block
    total = 0
    for b in range(p.blocks):
        seg = range(p.seg_ptr[b], p.seg_ptr[b + 1])
        ends = [(p.seg_row[s], p.seg_row[s] + p.seg_len[s]) for s in seg]
        assert all(hi0 < lo1 for (_, hi0), (lo1, _) in zip(ends, ends[1:]))   # sorted, disjoint, maximal
        window = np.concatenate([np.arange(lo, hi) for lo, hi in ends])
        e0, e1 = csr.rowptr[p.block_row[b]], csr.rowptr[p.block_row[b + 1]]
        assert np.array_equal(window[p.slot[e0:e1]], csr.col[e0:e1])
        assert set(window) == set(csr.col[e0:e1]) and len(window) <= p.max_window_rows <= cap
        assert e1 - e0 <= p.max_slice_nnz and p.block_row[b + 1] - p.block_row[b] <= p.max_block_rows
        total += len(window)
    assert max(p.seg_ptr[b + 1] - p.seg_ptr[b] for b in range(p.blocks)) >= segments
    assert p.amplification == total / csr.n_rows


def test_ring_amplification_by_hand():
    """A block of r ring rows reads r + 2 rows: blocks of 46 under a 48-row window, 300 = 6 x 46 +
    24, so (300 + 2 x 7) / 300."""
    from distributed_learning_amd.graph import band_blocks
    p = band_blocks(ring(300), 48)
    assert np.diff(p.block_row).tolist() == [46] * 6 + [24]
    assert p.amplification == 314 / 300


def test_no_locality_is_refused_and_bfs_order_restores_it():
    from distributed_learning_amd import graph
    rr = graph.uniform_weights(graph.random_regular_edges(4, 2000, 0), 0.2)
    with pytest.raises(ValueError, match="no locality"):
        graph.band_blocks(rr, 256)
    with pytest.raises(ValueError, match="alone"):
        graph.band_blocks(ring(300), 2)
    # a scattered numbering of the torus: refused as it stands, banded again in BFS order
    scat = graph.permuted(torus(12, 25), np.random.default_rng(1).permutation(300))
    with pytest.raises(ValueError, match="no locality"):
        graph.band_blocks(scat, 64, max_amplification=3.0)
    order = graph.bfs_order(scat)
    assert sorted(order.tolist()) == list(range(300))
    assert graph.band_blocks(graph.permuted(scat, order), 100, max_amplification=8.0).blocks > 1
