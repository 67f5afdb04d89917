"""What the float64 restatements of the all-pairs measures share (tests/domain_gap_reference.py, tests/tsne_reference.py,
tests/svc_reference.py): the squared distances by direct differences and the unit round-off of float32.  Plain numpy;
nothing here is shared with the product."""
import numpy as np

U = 2.0 ** -24                                          # unit round-off of float32


def d2_matrix(x):
    """(N, D) float32 -> (N, N) float64 squared distances by direct differences (exact differences of the float32
    values, float64 squares and sums)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    out = np.empty((x.shape[0], x.shape[0]))
    for i in range(x.shape[0]):
        diff = x - x[i]
        out[i] = np.einsum("nd,nd->n", diff, diff)
    return out
