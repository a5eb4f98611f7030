"""A self-check of the test suite's own restatement (tests/lcbext.py), not a test of the product: the line-by-line table that the
other modules compare the engine with is the cell-by-cell table that INTEGRATION.md 1e writes down.  It runs no engine code."""
import numpy as np

import lcbext as X


def test_table_restatement():
    """the line-by-line table is the cell-by-cell one of 1e"""
    rng = np.random.default_rng(5)
    for W, scores in ((1, (1, 1, 1)), (3, (5, 4, 2)), (7, (1, 1, 1)), (2, (2, 0, 3))):
        p = X.params(band=W, match=scores[0], mismatch=scores[1], gap=scores[2])
        for La, Lb in ((0, 0), (0, 3), (5, 0), (9, 14), (14, 9), (12, 12), (1, 30)):
            a = X.rand_seq(rng, La)
            b = X.mutate(rng, (a + X.rand_seq(rng, Lb))[:Lb], subs=min(2, Lb))
            slow, H = X.table_slow(a, b, p), X.table(a, b, p)
            ex = X.exists(H, p)
            assert set(slow) == {(int(i), int(j)) for i, j in np.argwhere(ex)}
            assert all(H[i, j] == v for (i, j), v in slow.items())
    p = X.params(band=2)
    assert list(X.best_of(X.table(b"ACGTACGT", b"ACG", p), p)) == [0, 5, 10, 15, 13, 11] + [X.UNDEF] * 3      # (lines 6 ... 8 have no cell)
    assert X.passes(10, 48, X.params()) and not X.passes(10, 45, X.params()) and not X.passes(3, X.UNDEF, X.params())
